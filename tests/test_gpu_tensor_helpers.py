"""GPU: the tensor helpers of the Python binding (compress_tensor / decompress_tensor of huffman, lz, arithmetic and layers, all over
_lib.dev_tensor) through every branch -- no `out`, an `out` that is exactly large enough (a view of it comes back), an `out` that is too
small (a fresh tensor, or for lz.compress_tensor the RsnError with .needed), and the size query that the Huffman and LZSS
decompress_tensor make from 1 MiB of stream up.  Expected bytes come from the host-buffer calls and the oracle."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = ["lzss", "huffman"]


@pytest.fixture(scope="module")
def ref(oracle):
    """the 4 KiB input, and per codec: (compress_tensor, decompress_tensor, the device entry points and their extras, the stream)"""
    from raisin_amd import _lib, arithmetic, huffman, layers, lz
    L = _lib.lib()
    sam = open(os.path.join(ROOT, "tests", "golden", "samiam.txt"), "rb").read()
    data = (sam * (4096 // len(sam) + 1))[:4096]
    arr, k = layers.ids(LAYERS)
    streams = {"huffman": huffman.Compress(data), "lzss": lz.CompressAsync(data, False, 4096), "arithmetic": arithmetic.Compress(data),
               "layers": layers.Compress(data, LAYERS)}
    assert streams["huffman"] == oracle.huffman_compress(data) and streams["lzss"] == oracle.lzss_compress(data, 4096)
    assert streams["layers"] == oracle.huffman_compress(oracle.lzss_compress(data, 4096))
    assert arithmetic.Decompress(streams["arithmetic"]) == data
    codecs = {
        "huffman": (huffman.compress_tensor, huffman.decompress_tensor, L.rsn_huffman_compress_dev, L.rsn_huffman_decompress_dev, ()),
        "lzss": (lz.compress_tensor, lz.decompress_tensor, L.rsn_lzss_compress_dev, L.rsn_lzss_decompress_dev, ()),
        "arithmetic": (arithmetic.compress_tensor, arithmetic.decompress_tensor, L.rsn_arithmetic_compress_dev, L.rsn_arithmetic_decompress_dev, ()),
        "layers": (lambda src, **kw: layers.compress_tensor(src, LAYERS, **kw), lambda src, **kw: layers.decompress_tensor(src, LAYERS, **kw),
                   L.rsn_layers_compress_dev, L.rsn_layers_decompress_dev, (arr, k)),
    }
    return data, streams, codecs


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _bytes(t):
    return bytes(t.cpu().numpy())


def _needed(fn, src, extra):
    """what the entry point itself asks for when 16 bytes are too few (not through the helper under test)"""
    import torch
    from raisin_amd import _lib
    small = torch.empty(16, dtype=torch.uint8, device="cuda")
    _lib.own_stream(src)
    if fn is _lib.lib().rsn_lzss_compress_dev:
        extra = (4096,)
    with pytest.raises(_lib.RsnError) as e:
        _lib.call_dev(fn, src.data_ptr(), src.numel(), small.data_ptr(), 16, None, *extra)
    assert e.value.code == _lib.RSN_ERR_CAPACITY and e.value.needed > 16
    return e.value.needed


@pytest.mark.parametrize("name", ["huffman", "lzss", "arithmetic", "layers"])
@pytest.mark.parametrize("direction", ["compress", "decompress"])
def test_every_branch_of_the_tensor_helpers(ref, name, direction):
    import torch
    from raisin_amd import _lib
    data, streams, codecs = ref
    comp, decomp, fn_c, fn_d, extra = codecs[name]
    helper, fn = (comp, fn_c) if direction == "compress" else (decomp, fn_d)
    given, want = (data, streams[name]) if direction == "compress" else (streams[name], data)
    src = _dev(given)
    assert _bytes(helper(src)) == want                                    # out=None
    exact = torch.empty(_needed(fn, src, extra), dtype=torch.uint8, device="cuda")
    got = helper(src, out=exact)
    assert got.data_ptr() == exact.data_ptr() and _bytes(got) == want     # large enough: a view of it
    small = torch.empty(16, dtype=torch.uint8, device="cuda")
    if name == "lzss" and direction == "compress":                        # the one helper that does not call again
        with pytest.raises(_lib.RsnError) as e:
            helper(src, out=small)
        assert e.value.code == -7 and e.value.needed >= len(want)
    else:
        got = helper(src, out=small)
        assert got.data_ptr() != small.data_ptr() and _bytes(got) == want   # too small: a fresh tensor


@pytest.mark.parametrize("name", ["huffman", "lzss"])
def test_the_size_query_from_one_mib_of_stream(name):
    """the smallest shape that reaches it: a stream just over 1 MiB (letters without repeats worth a token: LZSS leaves them as they
    are, Huffman takes them to 4.7 bits each)"""
    from raisin_amd import huffman, lz
    rng = np.random.default_rng(0x7E50)
    data = rng.integers(97, 123, size=((1 << 20) + 4096) * (2 if name == "huffman" else 1), dtype=np.uint8).tobytes()
    stream = huffman.Compress(data) if name == "huffman" else lz.CompressAsync(data, False, 4096)
    assert (1 << 20) <= len(stream) < (1 << 20) + (1 << 18)
    mod = huffman if name == "huffman" else lz
    assert mod.Decompress(stream) == data
    assert _bytes(mod.decompress_tensor(_dev(stream))) == data
