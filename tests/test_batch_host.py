"""The batch forms of Huffman decompress and LZSS compress / decompress (include/rsn.h): declared, exported and bound, and -- without a
device -- failing the way every codec entry point does, with every outs[i] left NULL.  Runs on any machine."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rsn_huffman_decompress_batch", "rsn_lzss_compress_batch", "rsn_lzss_decompress_batch")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from raisin_amd import _lib
    return _lib


def _call(L, name, bufs, ins=True, lens=True, outs=True, olens=True, window=4096):
    k = len(bufs)
    a_ins = (ctypes.c_char_p * k)(*bufs) if ins else None
    a_lens = (ctypes.c_size_t * k)(*[len(b) for b in bufs]) if lens else None
    a_outs = (ctypes.POINTER(ctypes.c_uint8) * k)() if outs else None
    a_olens = (ctypes.c_size_t * k)() if olens else None
    if outs:
        for i in range(k):                                  # garbage the call must overwrite with NULL
            a_outs[i] = ctypes.cast(ctypes.c_void_p(0x1000 + 16 * i), ctypes.POINTER(ctypes.c_uint8))
    extra = (window,) if name == "rsn_lzss_compress_batch" else ()
    rc = getattr(L, name)(k, a_ins, a_lens, *extra, a_outs, a_olens)
    return rc, a_outs


def test_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "rsn.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rsn_[a-z0-9_]+)\s*\(", hdr))
    L = built.lib()
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in built.SYMBOLS, name
        assert getattr(L, name).argtypes, name


def test_python_wrappers_exist(built):
    from raisin_amd import huffman, lz
    assert callable(huffman.DecompressBatch) and callable(lz.CompressAsyncBatch) and callable(lz.DecompressBatch)
    assert huffman.BATCH_GROUP_PAYLOAD_MAX == 16384 and huffman.BATCH_GROUP_OUTPUT_MAX == 32768


def test_null_arrays_are_refused(built):
    L = built.lib()
    bufs = [b"abc", b"de"]
    for name in NEW:
        for missing in ("ins", "lens", "outs", "olens"):
            rc, _ = _call(L, name, bufs, **{missing: False})
            assert rc == -1, (name, missing)
        # a null member with a non-zero length
        k = 2
        ins = (ctypes.c_char_p * k)(b"abc", None)
        lens = (ctypes.c_size_t * k)(3, 5)
        outs = (ctypes.POINTER(ctypes.c_uint8) * k)()
        olens = (ctypes.c_size_t * k)()
        extra = (4096,) if name == "rsn_lzss_compress_batch" else ()
        assert getattr(L, name)(k, ins, lens, *extra, outs, olens) == -1, name
        assert all(not outs[i] for i in range(k))


def test_empty_batch_is_ok(built):
    L = built.lib()
    for name in NEW:
        assert _call(L, name, [])[0] == 0, name
        extra = (4096,) if name == "rsn_lzss_compress_batch" else ()
        assert getattr(L, name)(0, None, None, *extra, None, None) == 0, name


def test_without_a_device_every_member_stays_null(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = built.lib()
    bufs = [b"Hello world!\n", b"", b"abcabcabcabcabcabcabcabc\n", b"x" * 5000]
    for name in NEW:
        rc, outs = _call(L, name, bufs)
        assert rc == -4, name
        assert b"no CPU fallback" in L.rsn_last_error(), name
        assert all(not outs[i] for i in range(len(bufs))), name
