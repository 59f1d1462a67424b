"""CPU tests of the layered calls (rsn_layers_*, include/rsn.h): argument errors are reported before a device is looked for, valid
arguments without a device fail loudly, and the Python mirror maps the engine's layer names."""
import ctypes

import pytest

LZSS, HUFFMAN = 1, 2


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from raisin_amd import _lib
    return _lib


def _ids(*v):
    return (ctypes.c_int * max(len(v), 1))(*v), len(v)


def _host_calls(L):
    return [L.rsn_layers_compress, L.rsn_layers_decompress]


def test_argument_errors_come_before_any_device(built):
    L = built.lib()
    data = b"abcabcabcabc\n"
    for fn in _host_calls(L):
        for arr, k, word in ((None, 2, b"null layer list"), (_ids(LZSS, 7)[0], 2, b"unknown layer id 7"), (_ids(0)[0], 1, b"unknown layer id 0"),
                             (_ids(*([LZSS, HUFFMAN] * 5))[0], 9, b"at most 8")):
            out = ctypes.POINTER(ctypes.c_uint8)()
            n = ctypes.c_size_t(5)
            assert fn(data, len(data), arr, k, ctypes.byref(out), ctypes.byref(n)) == -1
            assert word in L.rsn_last_error() and not out and n.value == 0
        arr, k = _ids(LZSS, HUFFMAN)
        assert fn(data, len(data), arr, k, None, None) == -1
    got = ctypes.c_size_t(0)
    for fn in (L.rsn_layers_compress_dev, L.rsn_layers_decompress_dev):
        assert fn(16, 16, None, 1, 4096, 64, ctypes.byref(got), None) == -1
        assert fn(16, 16, _ids(9)[0], 1, 4096, 64, ctypes.byref(got), None) == -1 and b"unknown layer id 9" in L.rsn_last_error()
        assert fn(16, 16, _ids(*([LZSS] * 9))[0], 9, 4096, 64, ctypes.byref(got), None) == -1
        assert fn(16, 16, _ids(LZSS)[0], 1, 4100, 64, ctypes.byref(got), None) == -1 and b"16-byte aligned" in L.rsn_last_error()
        assert fn(4096, 64, _ids(LZSS, HUFFMAN)[0], 2, 4096 + 32, 64, ctypes.byref(got), None) == -1 and b"overlap" in L.rsn_last_error()
    res = built.RoundTripResult()
    res.original_n = 77
    assert L.rsn_layers_roundtrip(data, len(data), None, 1, ctypes.byref(res), None, None) == -1
    assert res.original_n == 0                                            # left zeroed
    assert L.rsn_layers_roundtrip(data, len(data), _ids(3)[0], 1, ctypes.byref(res), None, None) == -1
    assert L.rsn_layers_roundtrip(data, len(data), _ids(LZSS)[0], 1, None, None, None) == -1


def test_valid_arguments_without_a_device_fail_loudly(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = built.lib()
    data = b"abcabcabcabc\n"
    for layers in ((), (LZSS,), (HUFFMAN,), (LZSS, HUFFMAN)):
        arr, k = _ids(*layers)
        for fn in _host_calls(L):
            out = ctypes.POINTER(ctypes.c_uint8)()
            n = ctypes.c_size_t(0)
            assert fn(data, len(data), arr, k, ctypes.byref(out), ctypes.byref(n)) == -4
            assert b"no CPU fallback" in L.rsn_last_error() and not out
        res = built.RoundTripResult()
        assert L.rsn_layers_roundtrip(data, len(data), arr, k, ctypes.byref(res), None, None) == -4
        assert b"no CPU fallback" in L.rsn_last_error() and res.original_n == 0
        got = ctypes.c_size_t(0)
        for fn in (L.rsn_layers_compress_dev, L.rsn_layers_decompress_dev):
            assert fn(4096, 16, arr, k, 8192, 4096, ctypes.byref(got), None) == -4 and b"no CPU fallback" in L.rsn_last_error()


def test_copy_counters_exist_and_start_at_zero(built):
    built.prof_enable(True)
    built.prof_reset()
    assert built.prof_copied() == (0, 0)
    built.prof_enable(False)
    assert built.prof_get() == {}                                         # the counters add no entry to rsn_prof_get


def test_python_mirror_maps_the_engines_names(built):
    from raisin_amd import RsnError, engine, layers
    arr, k = layers.ids(["lzss", "huffman", "lzss"])
    assert k == 3 and list(arr) == [LZSS, HUFFMAN, LZSS]
    assert layers.ids([])[1] == 0
    with pytest.raises(ValueError):
        layers.ids(["lzss", "arithmetic"])
    assert layers.LAYERS_MAX == 8 and set(layers.IDS) == set(engine.Engines)
    with pytest.raises(RsnError) as e:                                    # more than RSN_LAYERS_MAX in ONE call is the caller's to split
        layers.Compress(b"abc", ["lzss"] * 9)
    assert e.value.code == -1
    assert engine._on_device(["lzss", "huffman"]) and not engine._on_device(["lzss", "dmc"])
